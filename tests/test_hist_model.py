"""The byte-histogram model (tests/hist_model.py) against the oracle and the compiled reference: the histogram of a cloud's
stream is a sum of per-field terms, bin for bin; and its order-0 entropy against what the reference's ZSTD makes of the same
cloud. cldn_hip_hist_entropy_bytes (host only) against numpy. No GPU."""
import os

import numpy as np
import pytest

import cases
import hist_model as H
import sweep_model as S
from cloudini_amd import api, synth
from cloudini_amd.schema import CompressionOption

# every field a lossy float: sum of the fields' histograms + the prefix bytes == the stream's histogram
ABSOLUTE = [
    ("lidar_xyz_70000", lambda: synth.lidar_xyz(70000)),
    ("xyzi_struct_4133", cases.xyzi_struct_4133),
    ("five_floats", cases.five_floats),
    ("float_specials3", lambda: cases.float_specials(lanes=3)),
    ("float_specials4", lambda: cases.float_specials(lanes=4, seed=4)),
]

# integer sections or raw fields next to the lossy floats: what the stream holds beyond a field's tokens does not move with it
INCREMENTS = [
    ("velodyne_xyzir_40000", lambda: synth.velodyne_xyzir(40000)),
    ("depthcam_xyzrgba_320x240", lambda: synth.depthcam_xyzrgba(320, 240)),
    ("mixed_schema_float64_stamp", cases.mixed_schema),
    ("region_overflow3_u16", lambda: cases.region_overflow(lanes=3, seed=73, with_u16=True)),
]


def _with_resolution(info, f, r):
    out = info.copy()
    out.fields[f].resolution = float(np.float32(r))
    return out


def _payload_hist(stream):
    """The stream's histogram without the bytes of its [u32] prefixes: those spell the payload sizes, which move with a field."""
    return H.bytes_hist(stream).astype(np.int64) - H.prefix_hist(stream).astype(np.int64)


def _identities(encode, info, data, absolute):
    n = data.size // info.point_step
    kinds = S.field_kinds(info)
    ladders = S.default_ladders(info)
    rep = H.sweep_hist(info, data, [n], ladders)[0]
    base = encode(info, data)
    # the histograms hold the bytes the sweep counts
    assert np.array_equal(rep.sum(axis=2), S.sweep(info, data, [n], ladders)[0]["bytes"])
    if absolute:
        assert all(k != S.NONE for k in kinds)
        assert np.array_equal(rep[:, 0].sum(axis=0) + H.prefix_hist(base), H.bytes_hist(base))
    checked = 0
    for f, kind in enumerate(kinds):
        if kind == S.NONE:
            assert not rep[f].any()
            continue
        rest = _payload_hist(base) - rep[f, 0].astype(np.int64)
        assert (rest >= 0).all()
        for c, r in enumerate(ladders[f][1:], start=1):
            stream = encode(_with_resolution(info, f, r), data)
            assert np.array_equal(_payload_hist(stream) - rep[f, c].astype(np.int64), rest), (info.fields[f].name, float(r))
            checked += 1
    assert checked >= 4


@pytest.mark.parametrize("name,make", ABSOLUTE, ids=[c[0] for c in ABSOLUTE])
def test_sum_of_field_histograms_plus_prefixes_is_the_oracle_stream(oracle, name, make):
    info, data = make()
    _identities(oracle.encode_stage1, info, data, absolute=True)


@pytest.mark.parametrize("name,make", INCREMENTS, ids=[c[0] for c in INCREMENTS])
def test_moving_one_field_changes_the_oracle_stream_by_its_histograms(oracle, name, make):
    info, data = make()
    if name.startswith("mixed"):
        kinds = dict(zip([f.name for f in info.fields], S.field_kinds(info)))
        assert kinds["stamp"] == S.SCALAR64
    _identities(oracle.encode_stage1, info, data, absolute=False)


@pytest.mark.parametrize("name,make", [ABSOLUTE[1], INCREMENTS[0], INCREMENTS[2]], ids=["xyzi_struct_4133", "velodyne", "mixed"])
def test_the_same_against_the_compiled_reference(reflib, name, make):
    info, data = make()
    _identities(reflib.encode_stage1, info, data, absolute=name == "xyzi_struct_4133")


def test_token_bytes_of_every_length():
    """Bytes >= 0x80 and the top groups: tokens of 1..5 bytes in the int32 kind, 1..10 in the int64 kinds; the NaN marker; the
    wrapped int64 token."""
    u = np.array([1, 0x7F, 0x80, 0x3FFF, 0x4000, (1 << 28) - 1, 1 << 28, 1 << 32, (1 << 63), (1 << 64) - 1, 0], dtype=np.uint64)
    nan = np.zeros(u.size, dtype=bool)
    want = np.zeros(256, dtype=np.uint64)
    for x in u.tolist():
        while True:
            b = x & 0x7F
            x >>= 7
            want[b | (0x80 if x else 0)] += 1
            if not x:
                break
    assert np.array_equal(H.token_hist(u, nan), want) and int(want.sum()) == 1 + 1 + 2 + 2 + 3 + 4 + 5 + 5 + 10 + 10 + 1
    nan[:] = True
    assert H.token_hist(u, nan)[0] == u.size and H.token_hist(u, nan).sum() == u.size
    # the model through the quantisers: 100 -> zig-zag 200 + 1 = 201 = [0xC9, 0x01], then deltas of 0 -> 0x01; NaN -> 0x00
    v = np.array([100, 100, np.nan, 100, 100], dtype=np.float32)
    for kind in (S.FLOATN, S.SCALAR32):
        h = H.field_hist(kind, v, 1.0)
        assert h[0xC9] == 2 and h[0x01] == 4 and h[0x00] == 1 and h.sum() == 7
    # +-inf, and |v| / r beyond int32: the sentinel's delta fills the fifth byte of the int32 kind
    v = np.array([0.0, 3e9, 0.0, -np.inf, np.inf], dtype=np.float32)
    assert H.field_hist(S.FLOATN, v, 0.001).sum() == S.field_cell(S.FLOATN, v, 0.001)[0] > 5 + 5


# ---- the estimate against real ZSTD ------------------------------------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v1.npz")
# Measured (this test prints them): estimate / ZSTD payload over the five rungs of the default ladder, per slice
# of the reference's two sample files. lidar.pcd is XYZI float32, all tokens: the order-0 entropy is ZSTD's size within 2 %.
# dds_message.bin also carries a ring and a lossless float64 stamp (Gorilla): their bytes repeat, ZSTD's matches halve them,
# and an order-0 figure cannot see that -- the estimate is 1.9 to 2.05 times the file there. The assertion is each measured
# range widened by 0.05 on both sides: it catches a broken composition (a missing field, a double-counted one, the wrong
# rung), it does not certify ZSTD.
RATIOS = {"sample_lidar_pcd_8000": (0.985, 0.992), "sample_dds_message_6000": (1.880, 2.053)}
LIDAR_SLICES = list(RATIOS)


def _golden(name):
    z = np.load(GOLDEN)
    info = api.parse_yaml_info(z[name + "/yaml"].tobytes().decode(), int(z[name + "/version"][0]))
    info.use_threads = False
    return info, z[name + "/input"]


def estimate_ratios(oracle, reflib):
    out = []
    for name in LIDAR_SLICES:
        info, data = _golden(name)
        n = data.size // info.point_step
        kinds = S.field_kinds(info)
        ladders = S.default_ladders(info)
        rep = H.sweep_hist(info, data, [n], ladders)[0]
        base = oracle.encode_stage1(info, data)
        hist = H.bytes_hist(base)
        for c in range(ladders.shape[1]):
            rung = info.copy()
            cloud = hist
            for f, kind in enumerate(kinds):
                if kind != S.NONE:
                    rung.fields[f].resolution = float(ladders[f, c])
                    cloud = H.moved(cloud, rep[f, 0], rep[f, c])
            none = rung.copy()
            none.compression_opt = CompressionOption.NONE
            stage1 = reflib.encode_stage1(none, data)
            # the composition is exact but for the four prefix bytes per chunk, which spell the new payload sizes
            assert np.array_equal(cloud.astype(np.int64) - H.prefix_hist(base), _payload_hist(stage1)), (name, c)
            rung.compression_opt = CompressionOption.ZSTD
            actual = reflib.encode(rung, data).size - len(reflib.header(rung))
            est = H.entropy_bytes(cloud)
            out.append((name, c, stage1.size, actual, est, est / actual))
    return out


def test_estimate_against_the_references_zstd(oracle, reflib):
    rows = estimate_ratios(oracle, reflib)
    for name, c, stage1, actual, est, ratio in rows:
        print(f"{name} rung {c}: stage-1 {stage1} B, ZSTD {actual} B, estimate {est:.0f} B, ratio {ratio:.3f}")
    for name, c, stage1, actual, est, ratio in rows:
        assert RATIOS[name][0] - 0.05 <= ratio <= RATIOS[name][1] + 0.05, (name, c, ratio)
    # the estimate ranks the rungs as the files do
    for name in LIDAR_SLICES:
        mine = [r for r in rows if r[0] == name]
        assert np.argsort([r[3] for r in mine]).tolist() == np.argsort([r[4] for r in mine]).tolist(), name


# ---- the libraries -----------------------------------------------------------------------------------------------------

def test_libraries_export_the_histogram_entry_points():
    from cloudini_amd import native
    for name in ("cldn_hip_sweep_hist_clouds", "cldn_hip_sweep_hist_last_encode", "cldn_hip_stream_hist",
                 "cldn_hip_stream_hist_last_encode", "cldn_hip_hist_entropy_bytes"):
        assert hasattr(native.lib(), name), name
    for name in ("sweep_hist_clouds_host", "sweep_hist_clouds_device", "sweep_hist_last_encode", "stream_hist_host",
                 "stream_hist_device", "stream_hist_last_encode"):
        assert hasattr(native.Codec, name), name
    for name in ("sweep_hist", "stream_hist", "hist_entropy_bytes"):
        assert hasattr(api, name), name


def test_hist_entropy_bytes_matches_numpy():
    from cloudini_amd import native
    rs = np.random.RandomState(7)
    one = np.zeros(256, dtype=np.uint64)
    one[3] = 123456
    skewed = np.zeros(256, dtype=np.uint64)
    skewed[1:4] = [10 ** 9, 3 * 10 ** 8, 10 ** 7]
    skewed[0x80:] = rs.randint(0, 1000, 128)
    cases_ = {"empty": np.zeros(256, dtype=np.uint64), "one_bin": one, "uniform": np.full(256, 4096, dtype=np.uint64),
              "skewed": skewed, "random": rs.randint(0, 1 << 40, 256).astype(np.uint64), "single_byte": (np.arange(256) == 255).astype(np.uint64)}
    for name, h in cases_.items():
        got, want = native.hist_entropy_bytes(h), H.entropy_bytes(h)
        assert abs(got - want) <= 1e-12 * max(abs(want), 1e-300), (name, got, want)
    assert native.hist_entropy_bytes(cases_["empty"]) == 0.0 and native.hist_entropy_bytes(one) == 0.0
    assert native.hist_entropy_bytes(cases_["uniform"]) == 256 * 4096                     # 8 bits per byte: capped at N
    assert 0 < native.hist_entropy_bytes(skewed) < int(skewed.sum()) / 4
    with pytest.raises(ValueError):
        native.hist_entropy_bytes(np.zeros(255, np.uint64))
